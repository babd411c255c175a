// ref_gap — the edit script of ONE gap from the UNMODIFIED reference functions (TEST INFRASTRUCTURE ONLY).
//
// Includes the reference's utils.h and edit_script.h from where they lie and links its edlib object
// (oracle/Makefile.ref).  Follows the three branches of CEncoder::GetEditDist (encoder.cpp:1255-1283)
// by calling the reference's own get_edit_dist_on_seq_empty, find_edit_dist_with_edlib_ex,
// find_edit_dist_with_edlib_ex_odwr, find_edit_dist_with_edlib_ex_odwr_reverse and refactor_edit_script:
// what tests/golden/make_gapshapes.py records, and the oracle's orc_gap_script is pinned to.
//
// usage: ref_gap CASES
//   CASES  text, three lines a case: "<name> <where>" (where: 0 left flank, 1 inner gap, 2 right flank),
//          the reference part, the read part (letters ACGT; "-" for an empty sequence)
//   stdout one line a case: <name> <edit distance> <ref_offset> <script length> <script or "-">
#include "utils.h"
#include "edit_script.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

static read_t to_read(const std::string& s)
{
	read_t r;
	if (s != "-")
		for (char c : s)
		{
			const char* p = strchr("ACGT", c);
			if (!p || !c) { fprintf(stderr, "ref_gap: symbol '%c' is not one of ACGT\n", c); exit(2); }
			r.push_back((uint8_t)(p - "ACGT"));
		}
	r.push_back(255);                                   // guard, as every read_t carries (utils.h:372-376)
	return r;
}

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: ref_gap CASES\n"); return 2; }
	std::ifstream in(argv[1]);
	if (!in) { perror("ref_gap"); return 2; }
	std::string name, ref_s, enc_s; int where;
	while (in >> name >> where >> ref_s >> enc_s)
	{
		const read_t ref = to_read(ref_s), enc = to_read(enc_s);
		read_view refPart(ref), encPart(enc);
		EditDistRes ed; uint32_t ref_offset = 0;
		if (refPart.empty() || encPart.empty()) ed = get_edit_dist_on_seq_empty(refPart, encPart);
		else
		{
			const uint32_t max_flank = static_cast<uint32_t>(encPart.size() * 2);
			if (where == 0)
			{
				ed = find_edit_dist_with_edlib_ex_odwr_reverse(refPart, encPart, max_flank, ref_offset, EDLIB_MODE_SHW);
				refactor_edit_script(refPart.substr(ref_offset), encPart, ed.editScript);
				ed.editScript = std::string(ref_offset, 'D') + ed.editScript;
			}
			else if (where == 2)
			{
				uint32_t tmp;
				ed = find_edit_dist_with_edlib_ex_odwr(refPart.substr(0, max_flank), encPart, tmp, EDLIB_MODE_SHW);
				refactor_edit_script(refPart, encPart, ed.editScript);
			}
			else
			{
				ed = find_edit_dist_with_edlib_ex(refPart, encPart);
				refactor_edit_script(refPart, encPart, ed.editScript);
			}
		}
		printf("%s %u %u %zu %s\n", name.c_str(), ed.editDist, ref_offset, ed.editScript.size(), ed.editScript.empty() ? "-" : ed.editScript.c_str());
	}
	return 0;
}
