// cull_runs_check.cpp -- a stand-alone CPU program (tests/test_cull_runs_host.py and tools/cull_runs_count.py build and run it) around the
// run rule of squad-mortar-helper_amd/csrc/smh_cull_rule.h: the culling scans take a row's white annulus pixels by runs, two look-ups per
// run, and a run's units are the smallest cyclic interval of units about the byte codes of its two ends.
//
//   cull_runs_check check [mutant]   every check below: exit 0 when all pass.  With a mutant's name the rule under test is that mutant, and
//                                    some check has to fail (exit 1)
//   cull_runs_check codes T          the condensed table of threshold T as text: "windows lo0 hi0 lo1 hi1 chained runs0 runs1", then (2R+1)
//                                    rows of (2R+1) entries "ab" + the byte code in hex, a / b = 1 where the pixel lies in the outer / the
//                                    middle annulus ("00ff" is a pixel of no annulus) -- for the count tool
//
// check, for every threshold T = 1 .. 49, every annulus the run rule applies to (smh_cull_by_runs), every row of the table, every cell of
// 32 columns as the scans cut them (ox = -R + 32 j + [0, 32)) and every sub-run [i, j] of consecutive annulus pixels inside the cell --
// any of them is a run of some mask:
//   (a) soundness: the run's units contain the OR of its pixels' dense units (smh_cull_units);
//   (b) equality:  where no code of the run is 0xFF the run's units ARE the OR of the units its pixels' codes stand for -- what the walk
//                  pixel by pixel gives.  All of T = 15 is in this case;
//   (c) the predicate refuses exactly the annuli whose lower step is < 3, and each of the three it refuses while a middle annulus or a
//       table exists -- T = 24 (middle), T = 48 and 49 (outer) -- holds a sub-run for which (a) fails: the predicate is needed;
//   (d) the bit form: smh_cull_run_starts / smh_cull_run_ends and their pairing (smh_cull_word_units) over a whole word of white pixels,
//       ANDed with a cell's annulus mask, give the union over the word's runs as a loop over its bits finds them -- every single run, every
//       pair of runs, the alternating and the full words, 10^5 seeded random words, over the cells of T = 15 -- and at T = 15 that is the
//       union over the pixels.
// Mutants: first_code_alone, larger_interval, ff_as_a_range, runs_at_lower_step_1, runs_before_the_mask.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define SMH_CULL_CHAIN
#include "smh_cull_rule.h"

static const int R = 52, DIM = 2 * R + 1, NU = SMH_CULL_UNITS;
static const unsigned long long ALL = (1ull << NU) - 1ull;
enum Mutant { NONE, FIRST_CODE_ALONE, LARGER_INTERVAL, FF_AS_A_RANGE, RUNS_AT_LOWER_STEP_1, RUNS_BEFORE_THE_MASK };
static Mutant mutant = NONE;

static unsigned long long fold(unsigned long long acc) { return (acc | (acc >> NU)) & ALL; }

// a cyclic interval of l units from unit f on, unit by unit (the mutants' arithmetic: nothing here can overflow a shift)
static unsigned long long interval(int f, int l) {
	unsigned long long m = 0ull;
	for (int k = 0; k < l && k < NU; ++k) m |= 1ull << ((f + k) % NU);
	return m;
}

// the rule under test, folded
static unsigned long long run_units(uint32_t ca, uint32_t cb) {
	if (mutant == NONE || mutant == RUNS_AT_LOWER_STEP_1 || mutant == RUNS_BEFORE_THE_MASK) return fold(smh_cull_run_units(ca, cb));
	if (mutant == FIRST_CODE_ALONE) return fold(smh_cull_code_units(ca));
	if (mutant != FF_AS_A_RANGE && (ca == 0xFFu || cb == 0xFFu)) return ALL;
	const int fa = (int)(ca & 63u) % NU, na = (int)(ca >> 6) + 1, fb = (int)(cb & 63u) % NU, nb = (int)(cb >> 6) + 1;
	const int d = (fb - fa + NU) % NU, e = (NU - d) % NU;
	const int la = d + nb > na ? d + nb : na, lb = e + na > nb ? e + na : nb;
	const bool from_a = mutant == LARGER_INTERVAL ? la > lb : la <= lb;
	return interval(from_a ? fa : fb, from_a ? la : lb);
}
static bool by_runs(uint32_t T, int a) {
	if (mutant != RUNS_AT_LOWER_STEP_1) return smh_cull_by_runs(T, a);
	int lo, hi;
	return smh_cull_window(T, a, &lo, &hi) && lo >= 1;
}
// a cell's units from the word of its white pixels and its annulus mask
static unsigned long long word_units(uint32_t white, uint32_t mask, const uint8_t *codes) {
	if (mutant == NONE) return fold(smh_cull_word_units(white & mask, codes, true));
	uint32_t s, e;
	if (mutant == RUNS_BEFORE_THE_MASK) { s = smh_cull_run_starts(white, true) & mask; e = smh_cull_run_ends(white, true) & mask; }
	else { s = smh_cull_run_starts(white & mask, true); e = smh_cull_run_ends(white & mask, true); }
	unsigned long long acc = 0ull;
	while (s && e) {
		acc |= run_units(codes[__builtin_ctz(s)], codes[__builtin_ctz(e)]);
		s &= s - 1u; e &= e - 1u;
	}
	return acc;
}

struct Table {
	uint32_t T;
	bool in[2][DIM][DIM + 23];                 // (rows padded to four cells of 32 columns)
	uint8_t code[DIM][DIM + 23];
};
static std::vector<unsigned long long> dense_units;      // smh_cull_units of every offset: they do not depend on T

static void build(Table &t, uint32_t T) {
	if (dense_units.empty()) {
		dense_units.resize(DIM * DIM);
		for (int oy = -R; oy <= R; ++oy)
			for (int ox = -R; ox <= R; ++ox) dense_units[(oy + R) * DIM + ox + R] = smh_cull_units(ox, oy);
	}
	std::memset(&t, 0, sizeof t);
	t.T = T;
	for (int oy = -R; oy <= R; ++oy)
		for (int ox = -R; ox <= R; ++ox) {
			const unsigned long long e = smh_cull_entry(T, ox, oy);
			t.in[0][oy + R][ox + R] = (e & SMH_CULL_IN_OUTER) != 0;
			t.in[1][oy + R][ox + R] = (e & SMH_CULL_IN_MIDDLE) != 0;
			t.code[oy + R][ox + R] = e ? smh_cull_unit_code(e & ALL) : 0xFF;
		}
}

struct Tally { long long runs, bad_sound, bad_equal, with_ff; int ex[3]; };

// (a) and (b) over every sub-run of annulus a of the table, whether or not the predicate lets the rule at it
static Tally walk(const Table &t, int a) {
	Tally n = {0, 0, 0, 0, {0, 0, 0}};
	for (int row = 0; row < DIM; ++row)
		for (int c0 = 0; c0 < DIM; c0 += 32)
			for (int i = c0; i < c0 + 32 && i < DIM; ++i) {
				unsigned long long dense = 0ull, coded = 0ull;
				bool ff = false;
				for (int j = i; j < c0 + 32 && j < DIM && t.in[a][row][j]; ++j) {
					dense |= dense_units[row * DIM + j];
					coded |= fold(smh_cull_code_units(t.code[row][j]));
					ff = ff || t.code[row][j] == 0xFF;
					const unsigned long long u = run_units(t.code[row][i], t.code[row][j]);
					++n.runs;
					n.with_ff += ff;
					if ((u & dense) != dense) { if (!n.bad_sound++) { n.ex[0] = row - R; n.ex[1] = i - R; n.ex[2] = j - R; } }
					if (!ff && u != coded) ++n.bad_equal;
				}
			}
	return n;
}

static int check() {
	int failed = 0;
	static Table t;
	long long total = 0;
	for (uint32_t T = 1; T <= 49; ++T) {
		build(t, T);
		for (int a = 0; a < 2; ++a) {
			int lo, hi;
			const bool exists = smh_cull_window(T, a, &lo, &hi);
			if (by_runs(T, a) != (exists && lo >= 3) && mutant != RUNS_AT_LOWER_STEP_1) { std::printf("FAILED (c): the predicate at T = %u, annulus %d\n", T, a); failed = 1; }
			if (!exists) continue;
			const Tally n = walk(t, a);
			if (by_runs(T, a)) {
				total += n.runs;
				if (n.bad_sound) { std::printf("FAILED (a): T = %u, annulus %d [%d, %d]: %lld of %lld runs miss units of their pixels, e.g. row %d, ox %d .. %d\n", T, a, lo, hi, n.bad_sound, n.runs, n.ex[0], n.ex[1], n.ex[2]); failed = 1; }
				if (n.bad_equal) { std::printf("FAILED (b): T = %u, annulus %d: %lld runs without 0xFF differ from the union of their pixels' codes\n", T, a, n.bad_equal); failed = 1; }
				if (T == 15 && n.with_ff) { std::printf("FAILED (b): T = 15 has runs with the code 0xFF\n"); failed = 1; }
			} else {
				if (!n.bad_sound) { std::printf("FAILED (c): T = %u, annulus %d [%d, %d] is refused and holds no counter-example\n", T, a, lo, hi); failed = 1; }
				else std::printf("T = %u, annulus %d [%d, %d] (refused): %lld of %lld runs would miss units, e.g. row %d, ox %d .. %d\n", T, a, lo, hi, n.bad_sound, n.runs, n.ex[0], n.ex[1], n.ex[2]);
			}
			if (T == 15) std::printf("T = 15, annulus %d [%d, %d]: %lld runs\n", a, lo, hi, n.runs);
		}
	}
	{   // the refused annuli are the three the rule's text names
		const bool r = !smh_cull_by_runs(24, 1) && smh_cull_by_runs(24, 0) && !smh_cull_by_runs(48, 0) && !smh_cull_by_runs(49, 0) && smh_cull_by_runs(47, 0) && smh_cull_by_runs(23, 1) && smh_cull_by_runs(23, 0)
			&& !smh_cull_by_runs(25, 1) && !smh_cull_by_runs(48, 1) && smh_cull_mode(15) == (2u | SMH_CULL_MODE_RUNS_OUTER | SMH_CULL_MODE_RUNS_MIDDLE) && smh_cull_mode(24) == (2u | SMH_CULL_MODE_RUNS_OUTER)
			&& smh_cull_mode(25) == (1u | SMH_CULL_MODE_RUNS_OUTER) && smh_cull_mode(48) == 1u;
		if (!r && mutant != RUNS_AT_LOWER_STEP_1) { std::printf("FAILED (c): the predicate / smh_cull_mode at the thresholds 23, 24, 25, 47, 48, 49\n"); failed = 1; }
	}
	// (d) the bit form, on the cells of T = 15
	build(t, 15);
	long long words = 0, bad_bits = 0, bad_union = 0;
	uint32_t ex_word = 0;
	auto one = [&](uint32_t white, int a, int row, int c0) {
		uint32_t mask = 0;
		for (int k = 0; k < 32 && c0 + k < DIM; ++k) mask |= (uint32_t)t.in[a][row][c0 + k] << k;
		const uint8_t *codes = &t.code[row][c0];
		unsigned long long by_loop = 0ull, by_pixel = 0ull;
		const uint32_t hit = white & mask;
		for (int k = 0; k < 32; ++k) {
			if (!((hit >> k) & 1u)) continue;
			int j = k;
			while (j + 1 < 32 && ((hit >> (j + 1)) & 1u)) ++j;
			by_loop |= fold(smh_cull_run_units(codes[k], codes[j]));
			for (int q = k; q <= j; ++q) by_pixel |= fold(smh_cull_code_units(codes[q]));
			k = j;
		}
		const unsigned long long got = word_units(white, mask, codes);
		++words;
		if (got != by_loop) { if (!bad_bits++) ex_word = white; }
		if (by_loop != by_pixel) ++bad_union;
	};
	uint64_t rng = 0x9E3779B97F4A7C15ull;
	auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
	for (int a = 0; a < 2; ++a)
		for (int row = 0; row < DIM; ++row)
			for (int c0 = 0; c0 < DIM; c0 += 32) {
				for (int i = 0; i < 32; ++i)
					for (int j = i; j < 32; ++j) one((uint32_t)(((1ull << (j - i + 1)) - 1ull) << i), a, row, c0);
				one(0x55555555u, a, row, c0); one(0xAAAAAAAAu, a, row, c0); one(0xFFFFFFFFu, a, row, c0); one(0u, a, row, c0);
				one(0x33333333u, a, row, c0); one(0xCCCCCCCCu, a, row, c0); one(0x80000001u, a, row, c0);
			}
	const int pair_rows[] = {0, 3, 17, 33, 34, 52, 53, 71, 87, 104};   // top, the rows tangent to the annuli's edges, the start pixel's and its neighbour, bottom
	for (int a = 0; a < 2; ++a)
		for (int row : pair_rows)
			for (int c0 = 0; c0 < DIM; c0 += 32)
				for (int i = 0; i < 32; ++i)
					for (int j = i; j < 32; ++j)
						for (int k = j + 2; k < 32; ++k)
							for (int l = k; l < 32; ++l)
								one((uint32_t)((((1ull << (j - i + 1)) - 1ull) << i) | (((1ull << (l - k + 1)) - 1ull) << k)), a, row, c0);
	for (int n = 0; n < 100000; ++n) {
		const uint64_t v = next();
		uint32_t white = (uint32_t)v;
		if (n & 1) white &= (uint32_t)(next() >> 16) | (uint32_t)(next() >> 24);      // (and sparser words, with longer gaps)
		one(white, (int)((v >> 32) & 1u), (int)((v >> 33) % DIM), 32 * (int)((v >> 48) & 3u));
	}
	if (bad_bits) { std::printf("FAILED (d): %lld of %lld words: starts / ends / pairing differ from the runs a loop over the bits finds, e.g. white = %08x\n", bad_bits, words, ex_word); failed = 1; }
	if (bad_union) { std::printf("FAILED (d): %lld of %lld words at T = 15: the union over the runs is not the union over the pixels\n", bad_union, words); failed = 1; }
	if (!failed) std::printf("ok: %lld runs of the annuli the rule applies to, %lld words\n", total, words);
	return failed;
}

int main(int argc, char **argv) {
	if (argc >= 2 && !std::strcmp(argv[1], "check")) {
		if (argc >= 3) {
			const char *names[] = {"", "first_code_alone", "larger_interval", "ff_as_a_range", "runs_at_lower_step_1", "runs_before_the_mask"};
			for (int i = 1; i < 6; ++i)
				if (!std::strcmp(argv[2], names[i])) mutant = (Mutant)i;
			if (mutant == NONE) { std::fprintf(stderr, "no such mutant: %s\n", argv[2]); return 2; }
		}
		return check();
	}
	if (argc >= 3 && !std::strcmp(argv[1], "codes")) {
		const uint32_t T = (uint32_t)std::atoi(argv[2]);
		static Table t;
		build(t, T);
		int lo0, hi0, lo1 = 0, hi1 = 0;
		smh_cull_window(T, 0, &lo0, &hi0);
		const bool mid = smh_cull_window(T, 1, &lo1, &hi1);
		std::printf("windows %d %d %d %d %d %d %d\n", lo0, hi0, mid ? lo1 : 0, mid ? hi1 : 0, (int)smh_cull_chained(T), (int)smh_cull_by_runs(T, 0), (int)smh_cull_by_runs(T, 1));
		for (int row = 0; row < DIM; ++row) {
			for (int col = 0; col < DIM; ++col) std::printf("%d%d%02x ", (int)t.in[0][row][col], (int)t.in[1][row][col], (unsigned)t.code[row][col]);
			std::printf("\n");
		}
		return 0;
	}
	std::fprintf(stderr, "usage: cull_runs_check check [mutant] | codes T\n");
	return 2;
}
