// fastx_input.hpp — the input of the command-line compressor with the reader's semantics (src/colord/in_reads.cpp:62-226): FASTQ / FASTA /
// multi-line FASTA, plain or gzip, CR LF tolerated, blank lines skipped, '+' line empty or equal to the id.  A Reader hands out Chunks of whole
// reader packs; a plain FASTQ is mapped and indexed by several threads.  `colord_hip parse-check` (parse_check.cpp) prints digests of them.
#pragma once
#include "archive.hpp"
#include <hip/hip_runtime_api.h>
#include <zlib.h>
#include <algorithm>
#include <chrono>
#include <thread>
#include <sys/mman.h>
#include <fcntl.h>
#include <unistd.h>

inline void hipck(hipError_t e, const char* what) { if (e != hipSuccess) die(std::string(what) + ": " + hipGetErrorString(e)); }

// ---- input: one sequential pass that finds lines (memchr) and assigns them their role; bases / qualities / ids are appended to the
// ---- chunk under construction.  A chunk closes at the first reader-pack boundary at or after chunk_bases.
struct Chunk {
	uint8_t* bases = nullptr; uint8_t* quals = nullptr; uint64_t cap = 0, n = 0;       // pinned staging (ASCII)
	bool pinned = true;                                                                // (false: plain host memory — `parse-check`, which needs no GPU)
	uint8_t* get(uint64_t bytes) { uint8_t* p = nullptr; if (pinned) hipck(hipHostMalloc((void**)&p, bytes, hipHostMallocDefault), "hipHostMalloc"); else { p = (uint8_t*)malloc(bytes); if (!p) die("out of memory"); } return p; }
	void give(uint8_t* p) { if (!p) return; if (pinned) (void)hipHostFree(p); else free(p); }
	std::vector<uint64_t> off{ 0 }; std::vector<uint32_t> packs{ 0 }; uint64_t pack_acc = 0;
	std::vector<uint32_t> parts{ 0 }; uint64_t part_acc = 0;                           // coder parts (--part-symbols); == packs by default
	void reserve(uint64_t need, bool with_quals)
	{
		if (need <= cap) return;
		// (chunks close at the first pack boundary at or after their target: the ones to come are a few MB larger or smaller than the first, and
		// pinning a gigabyte takes 0.1-0.3 s — exact first sizes meant a second, larger pair of buffers a few chunks later: 2.7 s of the
		// reader's 3.1 s at 20 Gbases)
		uint64_t nc = std::max<uint64_t>(need + need / 32 + (16ull << 20), cap + cap / 2 + (1ull << 24));
		uint8_t* nb = get(nc);
		if (n) memcpy(nb, bases, n);
		give(bases);
		bases = nb;
		if (with_quals) { uint8_t* nq = get(nc); if (n) memcpy(nq, quals, n); give(quals); quals = nq; }
		cap = nc;
	}
	// the range of the quality bytes, when whoever filled the chunk has looked (the indexed reader's copy threads do, while the bytes pass
	// through their caches: the check used to be one thread's loop over a gigabyte per chunk, on the thread that feeds the GPU)
	uint8_t qlo = 255, qhi = 0; bool q_range = false;
	void clear() { n = 0; off.assign(1, 0); packs.assign(1, 0); pack_acc = 0; parts.assign(1, 0); part_acc = 0; qlo = 255; qhi = 0; q_range = false; }
	// (Phred+33 0..95: anything else would index past the coder's tables) — false: the input is refused
	bool quals_in_range(int threads = 8)
	{
		if (!quals || !n) return true;
		if (!q_range)
		{
			const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)threads, n >> 22));
			std::vector<uint8_t> lo(T, 255), hi(T, 0); std::vector<std::thread> th;
			for (int i = 0; i < T; ++i) th.emplace_back([&, i]() {
				uint8_t a = 255, b = 0; const uint8_t* q = quals;
				for (uint64_t x = n * (uint64_t)i / T, e = n * (uint64_t)(i + 1) / T; x < e; ++x) { a = q[x] < a ? q[x] : a; b = q[x] > b ? q[x] : b; }
				lo[i] = a; hi[i] = b;
			});
			for (auto& t : th) t.join();
			for (int i = 0; i < T; ++i) { qlo = std::min(qlo, lo[i]); qhi = std::max(qhi, hi[i]); }
			q_range = true;
		}
		return qlo >= 33 && qhi <= 33 + 95;
	}
	void release() { give(bases); give(quals); bases = quals = nullptr; cap = 0; }
	bool full(uint64_t target) const { return n >= target && pack_acc == 0 && off.size() > 1; }      // closes at the first pack boundary at or after `target` bases
};
struct Reader {
	gzFile g = nullptr; bool gz = false, fastq = true; uint64_t file_bytes = 0, total_bytes = 0, header_symbols = 0;
	// plain FASTQ: the file is mapped and its lines go straight from the mapping into the pinned chunk buffers (one copy; the
	// generic path below copies every byte three times through zlib's buffer and a line string)
	const uint8_t* map = nullptr; const uint8_t* mp = nullptr; const uint8_t* me = nullptr;
	std::vector<uint8_t> buf; size_t pos = 0, len = 0; bool eof = false;
	std::string line[4]; int which = 0;                          // FASTQ record under construction
	std::string fa_header, fa_seq; int fa_state = 0;            // FASTA: 0 header, 1 EOLs after header, 2 read, 3 EOLs after / inside read
	std::vector<uint8_t> ids, plus; std::vector<uint64_t> id_off{ 0 };
	uint64_t n_reads = 0, n_bases = 0;
	uint64_t part_symbols = 2u << 21;
	bool replay = false;                                         // a later pass over the same input (--stream-input): ids, counters and checks are those of the first
	// back to the first record: the chunks come again exactly as in the first pass (the reference reads its input twice as well,
	// compression.cpp:432,547-561)
	void rewind()
	{
		replay = true;
		if (map) { mp = map; rec_pos = 0; return; }
		if (gzrewind(g) != 0) die("cannot rewind the input");
		pos = len = 0; eof = false; which = 0; for (auto& l : line) l.clear();
		fa_header.clear(); fa_seq.clear(); fa_state = 0;
	}
	// plain FASTQ, several threads: the mapping is cut into byte ranges at record starts, every range is indexed by a thread of its own
	// (line ends by memchr, the reader's checks), then the chunks are filled from the index by parallel copies (index_mapped below)
	struct Rec { const uint8_t* id; const uint8_t* seq; const uint8_t* qual; uint32_t id_len, len; uint8_t plus_eq; };
	std::vector<Rec> recs; size_t rec_pos = 0; bool indexed = false; int threads = 1;
	double t_book = 0, t_copy = 0;                               // (-v: bookkeeping on the reader's thread, parallel copies)
	void open(const std::string& path)
	{
		FILE* probe = fopen(path.c_str(), "rb");
		if (!probe) die("cannot open file: " + path);
		unsigned char mg[2] = { 0, 0 }; const size_t got = fread(mg, 1, 2, probe);
		fseeko(probe, 0, SEEK_END); file_bytes = (uint64_t)ftello(probe); fclose(probe);
		gz = got == 2 && mg[0] == 0x1f && mg[1] == 0x8b;
		g = gzopen(path.c_str(), "rb");
		if (!g) die("cannot open file: " + path);
		gzbuffer(g, 1 << 22);
		buf.resize(1 << 25);
		fill();
		if (!len) die("file " + path + " is empty");
		if (buf[0] != '@' && buf[0] != '>') die("unknown file format (the first character must be '@' or '>')");      // in_reads.cpp:256-262
		fastq = buf[0] == '@';
		if (!gz && fastq && file_bytes && !getenv("COLORD_HIP_NO_MMAP"))
		{
			const int fd = ::open(path.c_str(), O_RDONLY);
			if (fd >= 0)
			{
				void* m = mmap(nullptr, file_bytes, PROT_READ, MAP_PRIVATE, fd, 0);
				::close(fd);
				if (m != MAP_FAILED) { (void)madvise(m, file_bytes, MADV_SEQUENTIAL); map = mp = (const uint8_t*)m; me = map + file_bytes; total_bytes = file_bytes; }
			}
		}
	}
	// one line of the mapping at cursor `c`: [a, b) without its end-of-line characters; lines end at '\n' or '\r', empty lines are skipped (in_reads.cpp:188-226)
	static bool next_line(const uint8_t*& c, const uint8_t* end, const uint8_t*& a, const uint8_t*& b, bool short_line)
	{
		while (c < end && (*c == '\n' || *c == '\r')) ++c;
		if (c >= end) return false;
		a = c;
		const uint8_t* q = (const uint8_t*)memchr(c, '\n', (size_t)(end - c));
		b = q ? q : end;
		c = q ? q + 1 : end;
		if (b > a && b[-1] == '\r') --b;
		if (short_line) { const uint8_t* r = (const uint8_t*)memchr(a, '\r', (size_t)(b - a)); if (r) { c = r + 1; b = r; } }   // (a lone '\r' ends a line too; in a sequence or quality line it is refused as a symbol / quality value)
		return true;
	}
	// One record at cursor `c` of the mapping, with the reader's rules (in_reads.cpp:79-92,188-226); "" = fine, else the reader's complaint.
	static const char* parse_record(const uint8_t*& c, const uint8_t* end, Rec& r, uint64_t& hdr_syms, bool& got)
	{
		auto line = [&](const uint8_t*& a, const uint8_t*& b, bool short_line) { return next_line(c, end, a, b, short_line); };
		const uint8_t *h0, *h1, *s0, *s1, *p0, *p1, *q0, *q1;
		got = false;
		if (!line(h0, h1, true)) return "";
		if (!line(s0, s1, false) || !line(p0, p1, true) || !line(q0, q1, false)) return "truncated FASTQ record at the end of the input";
		if (*h0 != '@') return "FASTQ record does not start with '@'";
		if (*p0 != '+') return "FASTQ record without '+' line";
		if (s1 - s0 != q1 - q0) return "sequence and quality lengths differ";
		const bool eq = p1 - p0 > 1;
		if (eq && ((p1 - p0) != (h1 - h0) || memcmp(p0 + 1, h0 + 1, (size_t)(h1 - h0 - 1)) != 0)) return "quality header not empty but different than read header";
		if ((uint64_t)(s1 - s0) >= (1ull << 32) || (uint64_t)(h1 - h0) >= (1ull << 32)) return "line longer than 4 Gi symbols";
		hdr_syms += (uint64_t)(h1 - h0) + (uint64_t)(p1 - p0);
		r = Rec{ h0 + 1, s0, q0, (uint32_t)(h1 - h0 - 1), (uint32_t)(s1 - s0), (uint8_t)(eq ? 1 : 0) };
		got = true;
		return "";
	}
	// Index of the whole mapping by `threads` threads.  A range starts at the first line at or after its byte offset that begins with
	// '@', is followed two lines later by a '+' line and whose sequence and quality lines are equally long.  That is a guess (a quality
	// line may begin with '@'), so it is VERIFIED: the thread before must end its last record exactly there.  Any complaint or
	// mismatch: the index is dropped and the sequential reader (which reports errors in file order) takes over.
	bool index_mapped()
	{
		const int T = threads;
		const char* mn = getenv("COLORD_HIP_INDEX_MIN_BYTES");                        // (tests index small files too)
		if (T < 2 || (uint64_t)(me - map) < (mn ? strtoull(mn, nullptr, 10) : (64ull << 20))) return false;
		std::vector<const uint8_t*> b((size_t)T + 1, me);
		b[0] = map;
		for (int i = 1; i < T; ++i)
		{
			const uint8_t* p = map + (uint64_t)(me - map) * i / T;
			const uint8_t* q = (const uint8_t*)memchr(p, '\n', (size_t)(me - p));
			const uint8_t* found = nullptr;
			for (int tries = 0; q && tries < 64 && !found; ++tries)
			{
				const uint8_t* c = q + 1;
				while (c < me && (*c == '\n' || *c == '\r')) ++c;
				if (c >= me) break;
				if (*c == '@')
				{
					const uint8_t* cc = c; Rec r; uint64_t hs = 0; bool got = false;
					if (parse_record(cc, me, r, hs, got)[0] == 0 && got) { const uint8_t* n2 = cc; while (n2 < me && (*n2 == '\n' || *n2 == '\r')) ++n2; if (n2 >= me || *n2 == '@') found = c; }
				}
				q = (const uint8_t*)memchr(c, '\n', (size_t)(me - c));
			}
			if (!found) return false;
			b[i] = found;
		}
		for (int i = 1; i <= T; ++i) if (b[i] < b[i - 1]) return false;
		std::vector<std::vector<Rec>> part((size_t)T); std::vector<uint64_t> hs((size_t)T, 0); std::vector<int> bad((size_t)T, 0);
		std::vector<std::thread> th;
		for (int i = 0; i < T; ++i) th.emplace_back([&, i]() {
			const uint8_t* c = b[i]; const uint8_t* const stop = b[i + 1];
			part[i].reserve((size_t)((stop - c) / 20000 + 1024));
			for (;;)
			{
				while (c < me && (*c == '\n' || *c == '\r')) ++c;                       // (blank lines between records belong to nobody)
				if (c >= stop) break;
				Rec r; bool got = false;
				if (parse_record(c, me, r, hs[i], got)[0] != 0) { bad[i] = 1; return; }
				if (!got) break;
				part[i].push_back(r);
			}
			while (c < me && (*c == '\n' || *c == '\r')) ++c;
			const uint8_t* want = stop; while (want < me && (*want == '\n' || *want == '\r')) ++want;
			if (c != want) bad[i] = 1;                                                  // the next range does not begin where this one's last record ends
		});
		for (auto& t : th) t.join();
		for (int i = 0; i < T; ++i) if (bad[i]) return false;
		size_t total = 0; for (auto& v : part) total += v.size();
		recs.reserve(total);
		for (int i = 0; i < T; ++i) { recs.insert(recs.end(), part[i].begin(), part[i].end()); header_symbols += hs[i]; std::vector<Rec>().swap(part[i]); }
		indexed = true;
		return true;
	}
	// a chunk from the index: the bookkeeping (offsets, packs, parts, ids) in file order on this thread, the bases and qualities by parallel copies
	bool next_chunk_indexed(Chunk& ch, uint64_t target)
	{
		ch.clear();
		const size_t first = rec_pos;
		const auto tb0 = std::chrono::steady_clock::now();
		while (rec_pos < recs.size() && !ch.full(target))
		{
			const Rec& r = recs[rec_pos++];
			if (!replay) { ids.insert(ids.end(), r.id, r.id + r.id_len); id_off.push_back(ids.size()); plus.push_back(r.plus_eq); ++n_reads; n_bases += r.len; }
			ch.n += r.len; ch.off.push_back(ch.n);
			close_bounds(ch, r.len);
		}
		finish_bounds(ch);
		if (ch.off.size() <= 1) return false;
		{ const uint64_t total = ch.n; ch.n = 0; ch.reserve(total + 1, true); ch.n = total; }     // (nothing to carry over: the buffers are filled below)
		const size_t cnt = rec_pos - first; const int T = (int)std::min<size_t>((size_t)threads, std::max<size_t>(1, cnt / 256));
		const auto tb1 = std::chrono::steady_clock::now(); t_book += std::chrono::duration<double>(tb1 - tb0).count();
		std::vector<std::thread> th; std::vector<uint8_t> qmin(T, 255), qmax(T, 0);
		for (int i = 0; i < T; ++i) th.emplace_back([&, i]() {
			// (equal shares of the chunk's bytes: the offsets are ascending)
			const uint64_t lo_b = ch.n * (uint64_t)i / T, hi_b = ch.n * (uint64_t)(i + 1) / T;
			size_t lo = (size_t)(std::lower_bound(ch.off.begin(), ch.off.end() - 1, lo_b) - ch.off.begin());
			size_t hi = i + 1 == T ? cnt : (size_t)(std::lower_bound(ch.off.begin(), ch.off.end() - 1, hi_b) - ch.off.begin());
			uint8_t a = 255, b = 0;
			for (size_t x = lo; x < hi; ++x)
			{
				const Rec& r = recs[first + x];
				memcpy(ch.bases + ch.off[x], r.seq, r.len); memcpy(ch.quals + ch.off[x], r.qual, r.len);      // (pread() instead of the mapping: 0.8 against 0.5 s per 20 Gbases, profiles/r06_m_*)
				const uint8_t* q = (const uint8_t*)r.qual;                           // (the range of the quality bytes while they are in this core's cache)
				for (uint32_t y = 0; y < r.len; ++y) { a = q[y] < a ? q[y] : a; b = q[y] > b ? q[y] : b; }
			}
			qmin[i] = a; qmax[i] = b;
		});
		for (auto& t : th) t.join();
		t_copy += std::chrono::duration<double>(std::chrono::steady_clock::now() - tb1).count();
		for (int i = 0; i < T; ++i) { ch.qlo = std::min(ch.qlo, qmin[i]); ch.qhi = std::max(ch.qhi, qmax[i]); }
		ch.q_range = true;
		return true;
	}
	// pack / part bookkeeping of one more read of `len` symbols: a pack closes once its reads (with one guard byte each) reach 4 Mi
	// symbols (in_reads.cpp:62-77); the coder parts likewise at --part-symbols
	void close_bounds(Chunk& ch, uint64_t len)
	{
		ch.pack_acc += len + 1;
		if (ch.pack_acc >= (2u << 21)) { ch.packs.push_back((uint32_t)(ch.off.size() - 1)); ch.pack_acc = 0; }
		ch.part_acc += len + 1;
		if (ch.part_acc >= part_symbols) { ch.parts.push_back((uint32_t)(ch.off.size() - 1)); ch.part_acc = 0; }
	}
	void finish_bounds(Chunk& ch)
	{
		if (ch.off.size() > 1 && ch.packs.back() != ch.off.size() - 1) { ch.packs.push_back((uint32_t)(ch.off.size() - 1)); ch.pack_acc = 0; }
		if (ch.off.size() > 1 && ch.parts.back() != ch.off.size() - 1) { ch.parts.push_back((uint32_t)(ch.off.size() - 1)); ch.part_acc = 0; }
		if (part_symbols == (2u << 21)) ch.parts = ch.packs;
	}
	bool next_chunk_mapped(Chunk& ch, uint64_t target)
	{
		if (indexed) return next_chunk_indexed(ch, target);
		ch.clear();
		while (!ch.full(target))
		{
			const uint8_t *h0, *h1, *s0, *s1, *p0, *p1, *q0, *q1;
			if (!next_line(mp, me, h0, h1, true)) break;
			if (!next_line(mp, me, s0, s1, false) || !next_line(mp, me, p0, p1, true) || !next_line(mp, me, q0, q1, false)) die("truncated FASTQ record at the end of the input");
			if (*h0 != '@') die("FASTQ record does not start with '@'");
			if (*p0 != '+') die("FASTQ record without '+' line");
			if (s1 - s0 != q1 - q0) die("sequence and quality lengths differ");
			if (!replay) header_symbols += (uint64_t)(h1 - h0) + (uint64_t)(p1 - p0);
			const bool eq = p1 - p0 > 1;
			if (eq && ((p1 - p0) != (h1 - h0) || memcmp(p0 + 1, h0 + 1, (size_t)(h1 - h0 - 1)) != 0)) die("quality header not empty but different than read header");   // in_reads.cpp:79-92
			add_record(ch, (const char*)h0 + 1, (size_t)(h1 - h0 - 1), (const char*)s0, (size_t)(s1 - s0), (const char*)q0, eq);
		}
		finish_bounds(ch);
		return ch.off.size() > 1;
	}
	void fill() { const int n = gzread(g, buf.data(), (unsigned)buf.size()); if (n < 0) die("read error (zlib)"); len = (size_t)n; pos = 0; if (!replay) total_bytes += len; if (!n) eof = true; }
	void add_record(Chunk& ch, const char* id, size_t id_len, const char* seq, size_t seq_len, const char* qual, bool plus_eq)
	{
		if (!replay) { ids.insert(ids.end(), id, id + id_len); id_off.push_back(ids.size()); plus.push_back(plus_eq ? 1 : 0); ++n_reads; n_bases += seq_len; }
		ch.reserve(ch.n + seq_len + 1, fastq);
		memcpy(ch.bases + ch.n, seq, seq_len);
		if (fastq) memcpy(ch.quals + ch.n, qual, seq_len);
		ch.n += seq_len; ch.off.push_back(ch.n);
		close_bounds(ch, seq_len);
	}
	void flush_fastq(Chunk& ch)
	{
		if (line[0].empty() || line[0][0] != '@') die("FASTQ record does not start with '@'");
		if (line[2].empty() || line[2][0] != '+') die("FASTQ record without '+' line");
		if (line[1].size() != line[3].size()) die("sequence and quality lengths differ");
		if (!replay) header_symbols += line[0].size() + line[2].size();
		const bool eq = line[2].size() > 1;
		if (eq && line[2].compare(1, std::string::npos, line[0], 1, std::string::npos) != 0) die("quality header not empty but different than read header");   // in_reads.cpp:79-92
		add_record(ch, line[0].data() + 1, line[0].size() - 1, line[1].data(), line[1].size(), line[3].data(), eq);
	}
	void flush_fasta(Chunk& ch)
	{
		if (!replay) header_symbols += fa_header.size();
		add_record(ch, fa_header.data() + 1, fa_header.size() - 1, fa_seq.data(), fa_seq.size(), nullptr, false);
		fa_header.clear(); fa_seq.clear();
	}
	// fills `ch` up to the first pack boundary at or after `target` bases; returns false when the input is exhausted and ch is empty
	bool next_chunk(Chunk& ch, uint64_t target)
	{
		if (map) return next_chunk_mapped(ch, target);
		ch.clear();
		while (!eof && !ch.full(target))
		{
			if (pos >= len) { fill(); if (eof) break; }
			if (fastq)
			{	// lines end at '\n' or '\r'; empty lines are skipped (in_reads.cpp:188-226)
				const uint8_t* p = buf.data() + pos; const uint8_t* e = buf.data() + len;
				const uint8_t* q = (const uint8_t*)memchr(p, '\n', (size_t)(e - p)); const uint8_t* lim = q ? q : e;
				const uint8_t* r = (const uint8_t*)memchr(p, '\r', (size_t)(lim - p)); const uint8_t* nl = r ? r : lim;
				line[which].append((const char*)p, (size_t)(nl - p));
				pos = (size_t)(nl - buf.data());
				if (nl < e)
				{
					++pos;
					if (!line[which].empty()) { if (++which == 4) { flush_fastq(ch); which = 0; for (auto& l : line) l.clear(); } }
				}
			}
			else
			{	// porcessFastaOrMultiFasta (in_reads.cpp:114-178)
				for (; pos < len && !ch.full(target); ++pos)
				{
					const uint8_t s = buf[pos]; const bool eol = s == '\n' || s == '\r';
					switch (fa_state)
					{
					case 0: if (eol) fa_state = 1; else fa_header.push_back((char)s); break;
					case 1: if (!eol) { fa_seq.push_back((char)s); fa_state = 2; } break;
					case 2: if (eol) fa_state = 3; else fa_seq.push_back((char)s); break;
					case 3: if (!eol) { if (s == '>') { flush_fasta(ch); fa_state = 0; fa_header.push_back((char)s); } else { fa_state = 2; fa_seq.push_back((char)s); } } break;
					}
				}
			}
		}
		if (eof)
		{
			if (fastq) { if (!line[which].empty()) { if (++which == 4) { flush_fastq(ch); which = 0; for (auto& l : line) l.clear(); } } if (which != 0) die("truncated FASTQ record at the end of the input"); }
			else if (!fa_header.empty()) flush_fasta(ch);
		}
		finish_bounds(ch);
		return ch.off.size() > 1;
	}
};
