// cull_rule_check.cpp -- a stand-alone CPU program (tests/test_cull_chain_host.py and tools/cull_chain_count.py build and run it) around
// the sector culling rule of squad-mortar-helper_amd/csrc/smh_cull_rule.h.
//
//   cull_rule_check check       what the rule's pieces must mean, for every threshold T = 1 .. 49: exit 0 when every check passes
//   cull_rule_check table T     the dense table of threshold T as text: "windows lo0 hi0 lo1 hi1 chained", then (2R+1) rows of (2R+1)
//                               entries in hex (smh_cull_entry: units | annulus flags), R = 52 -- for the tests that hold the table against
//                               what rays sample and for the count tool
//
// check:
//   * the outer window is [50 - T, 50]; the middle one is [50 - 2T - 1, 50 - T - 1] and exists exactly where its lower end is >= 1; both
//     have T + 1 steps, they are disjoint and adjacent, and neither reaches beyond step 50 (a + T <= 50 is what the argument needs)
//   * an entry carries an annulus flag exactly where smh_cull_in_annulus says so for that window, units exactly where it carries a flag,
//     and the same units whichever annulus the pixel lies in; every pixel that can be sampled at a step <= 50 lies within R of the start
//   * smh_cull_live: the AND per unit where chained, the outer units alone where not
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "smh_cull_rule.h"

static const int R = 52;

static int fail(const char *what, unsigned T, int ox, int oy) {
	std::printf("FAILED: %s: T = %u, offset (%d, %d)\n", what, T, ox, oy);
	return 1;
}

static int check() {
	long long n = 0;
	for (unsigned T = 1; T <= 49; ++T) {
		int lo0, hi0, lo1, hi1;
		if (!smh_cull_window(T, 0, &lo0, &hi0) || lo0 != 50 - (int)T || hi0 != 50) return fail("the outer window", T, 0, 0);
		const bool mid = smh_cull_window(T, 1, &lo1, &hi1);
#ifdef SMH_CULL_CHAIN
		if (mid != (50 - 2 * (int)T - 1 >= 1)) return fail("where the middle window exists", T, 0, 0);
#else
		if (mid) return fail("a middle window in a build without the chain", T, 0, 0);
#endif
		if (mid != smh_cull_chained(T)) return fail("smh_cull_chained", T, 0, 0);
		if (mid && (lo1 != 50 - 2 * (int)T - 1 || hi1 != 50 - (int)T - 1 || hi1 - lo1 != (int)T || hi1 + 1 != lo0 || lo1 < 1)) return fail("the middle window", T, 0, 0);
		int lo2, hi2;
		if (smh_cull_window(T, 2, &lo2, &hi2)) return fail("a third window", T, 0, 0);
		for (int oy = -R - 2; oy <= R + 2; ++oy)
			for (int ox = -R - 2; ox <= R + 2; ++ox) {
				const unsigned long long e = smh_cull_entry(T, ox, oy), units = e & ((1ull << SMH_CULL_UNITS) - 1ull);
				const bool in0 = smh_cull_in_annulus(lo0, hi0, ox, oy), in1 = mid && smh_cull_in_annulus(lo1, hi1, ox, oy);
				++n;
				if (((e & SMH_CULL_IN_OUTER) != 0) != in0 || ((e & SMH_CULL_IN_MIDDLE) != 0) != in1) return fail("an entry's annulus flags", T, ox, oy);
				if ((units != 0) != (in0 || in1) || (e & ~(SMH_CULL_IN_OUTER | SMH_CULL_IN_MIDDLE)) != units) return fail("an entry's units", T, ox, oy);
				if ((in0 || in1) && units != smh_cull_units(ox, oy)) return fail("an entry's units depend on the annulus", T, ox, oy);
				if ((in0 || in1) && (std::abs(ox) > R || std::abs(oy) > R)) return fail("a pixel of an annulus beyond the table", T, ox, oy);
			}
	}
	const unsigned long long a = 0x0000F0F0ull, b = 0x0000FF00ull;
	if (smh_cull_live(a, b, true) != (a & b) || smh_cull_live(a, b, false) != a || smh_cull_live(a, 0ull, true) != 0ull || smh_cull_live(1ull, 2ull, true) != 0ull)
		return fail("smh_cull_live", 0, 0, 0);
	std::printf("ok: %lld entries checked\n", n);
	return 0;
}

int main(int argc, char **argv) {
	if (argc >= 2 && !std::strcmp(argv[1], "check")) return check();
	if (argc >= 3 && !std::strcmp(argv[1], "table")) {
		const unsigned T = (unsigned)std::atoi(argv[2]);
		int lo0, hi0, lo1 = 0, hi1 = 0;
		smh_cull_window(T, 0, &lo0, &hi0);
		const bool mid = smh_cull_window(T, 1, &lo1, &hi1);
		std::printf("windows %d %d %d %d %d\n", lo0, hi0, mid ? lo1 : 0, mid ? hi1 : 0, (int)smh_cull_chained(T));
		for (int oy = -R; oy <= R; ++oy) {
			for (int ox = -R; ox <= R; ++ox) std::printf("%llx ", smh_cull_entry(T, ox, oy));
			std::printf("\n");
		}
		return 0;
	}
	std::fprintf(stderr, "usage: cull_rule_check check | table T\n");
	return 2;
}
