// smh_cull_rule.h -- the sector culling rule of the line search: which 64-ray units of a candidate have to be cast at all
// (k_build_sector_table, smh_lsd.hip; the host's condensing code, smh_runtime.cpp; tests/cull_rule_check.cpp on the CPU.
// Host and device, no other header needed).
//
// lsd.rs:94 keeps a candidate only if its longest ray has len^2 > 2500, i.e. the ray's fatal gap starts at step K >= 51 (an
// aborted ray ends K - 1 unit steps from its start), or the ray leaves the image after more than 50 steps.  A ray is aborted
// by its (T + 1)-th consecutive non-white sample, T = ceil(max_gap).  So a ray that can be accepted has a WHITE sample in
// EVERY window of T + 1 consecutive steps [a, a + T] with a + T <= 50: a white-free window would have aborted it with K <= a.
// The windows [50 - T, 50] (the OUTER annulus) and [50 - 2T - 1, 50 - T - 1] (the MIDDLE annulus, where its lower end is
// >= 1) are disjoint, and each is a necessary condition on the same ray.  A ray lies in one unit, so a unit has to be cast
// only if it can see a white pixel in the outer annulus AND one in the middle annulus: the longest ray, if it is acceptable,
// lies in such a unit, and if no ray is acceptable the candidate is rejected whatever the other rays do.  (A third window,
// [3, 18] for T = 15, was counted on the benchmark's scene and removes no further unit: it stays out.)
//
// The build applies the OUTER annulus alone unless it is compiled with -DSMH_CULL_CHAIN: the chain leaves 17 % fewer units on the
// benchmark's scene (tools/cull_chain_count.py), but the scan of the second ring of pixels costs the search service more than
// those units do -- pixel by pixel, and by runs (below) as well -- so it is kept, checked and counted, and
// not used.  SMH_CULL_ANNULI is what the table holds and the kernels scan.
//
// The table maps a pixel offset (ox, oy) from floor(start point) to the units that could sample it, conservatively: the
// sample may sit anywhere in its pixel (0.71 px), the start point anywhere in its pixel (0.71 px), plus 0.05 px for
// accumulated f32 rounding -- rho.  A pixel at distance r0 is sampled at step k only if |r0 - k| <= rho, and only by rays
// within asin(rho / r0) of its direction (+ 0.2 degrees, two ray steps).  A pixel's units do not depend on the annulus it
// lies in; a pixel within rho of the boundary between the two belongs to both.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMH_CR_FN __host__ __device__ inline
#else
#define SMH_CR_FN inline
#endif

#define SMH_CULL_ACCEPT_STEP 50         // len^2 > 2500: the fatal gap starts after this step
#define SMH_CULL_UNITS 57               // 64-ray units of the 3600 rays (6.4 degree sectors)
#define SMH_CULL_RHO (0.7072 + 0.7072 + 0.05)
#define SMH_CULL_DELTA_MARGIN 0.2       // degrees
#define SMH_CULL_IN_OUTER (1ull << 62)  // dense table entry: the pixel lies in the outer / the middle annulus (units: bits 0 .. 56)
#define SMH_CULL_IN_MIDDLE (1ull << 63)
#ifdef SMH_CULL_CHAIN
#define SMH_CULL_ANNULI 2
#else
#define SMH_CULL_ANNULI 1
#endif

// Annulus `a` (0: outer, 1: middle) of threshold T: the steps [*lo, *hi].  false: there is no such annulus.
SMH_CR_FN bool smh_cull_window(uint32_t T, int a, int *lo, int *hi) {
	const int t = (int)T, top = SMH_CULL_ACCEPT_STEP - a * (t + 1);
	*hi = top;
	*lo = top - t < 0 ? 0 : top - t;
	if (a == 0) return true;
#ifdef SMH_CULL_CHAIN
	return a == 1 && top - t >= 1;
#else
	return false;
#endif
}
SMH_CR_FN bool smh_cull_chained(uint32_t T) { int lo, hi; return smh_cull_window(T, 1, &lo, &hi); }

// Can a sample at a step in [lo, hi] fall into the pixel at offset (ox, oy)?
SMH_CR_FN bool smh_cull_in_annulus(int lo, int hi, int ox, int oy) {
	const double r0 = sqrt((double)(ox * ox + oy * oy));
	return r0 >= (double)lo - SMH_CULL_RHO && r0 <= (double)hi + SMH_CULL_RHO;
}

// The units whose rays can sample the pixel at offset (ox, oy): ray i points at (cos, sin)(i / 10 degrees), y down.
SMH_CR_FN unsigned long long smh_cull_units(int ox, int oy) {
	const double rho = SMH_CULL_RHO;
	const double r0 = sqrt((double)(ox * ox + oy * oy));
	if (r0 <= rho) return (1ull << SMH_CULL_UNITS) - 1ull;              // the start pixel's neighbourhood: every direction
	const double PI = 3.14159265358979323846;
	double phi = atan2((double)oy, (double)ox) * 180.0 / PI;
	if (phi < 0.0) phi += 360.0;
	const double delta = asin(rho / r0 > 1.0 ? 1.0 : rho / r0) * 180.0 / PI + SMH_CULL_DELTA_MARGIN;
	unsigned long long m = 0ull;
	for (int u = 0; u < SMH_CULL_UNITS; ++u) {
		const double a0 = 6.4 * u, a1 = 6.4 * u + 6.3;                   // rays 64u .. 64u+63
		bool hit = false;                                               // intersects [phi - delta, phi + delta] modulo 360?
		for (int wrap = -1; wrap <= 1 && !hit; ++wrap) {
			const double lo = phi - delta + 360.0 * wrap, hi = phi + delta + 360.0 * wrap;
			hit = !(hi < a0 || lo > a1);
		}
		if (hit) m |= 1ull << u;
	}
	return m;
}

// The dense table's entry of offset (ox, oy) for threshold T: its units and the annuli it lies in; 0 outside both.
SMH_CR_FN unsigned long long smh_cull_entry(uint32_t T, int ox, int oy) {
	unsigned long long in = 0ull;
	int lo, hi;
	if (smh_cull_window(T, 0, &lo, &hi) && smh_cull_in_annulus(lo, hi, ox, oy)) in |= SMH_CULL_IN_OUTER;
	if (smh_cull_window(T, 1, &lo, &hi) && smh_cull_in_annulus(lo, hi, ox, oy)) in |= SMH_CULL_IN_MIDDLE;
	return in ? in | smh_cull_units(ox, oy) : 0ull;
}

// The unit test: the units white pixels of the outer annulus can be seen by, those of the middle annulus -> the units to cast.
// The AND is per unit: both pixels have to be seen by the SAME unit, since both conditions speak of one ray.
SMH_CR_FN unsigned long long smh_cull_live(unsigned long long seen_outer, unsigned long long seen_middle, bool chained) {
	return chained ? seen_outer & seen_middle : seen_outer;
}

// ---- a row's white pixels by runs ------------------------------------------------------------------------------------------
// The condensed table (smh_runtime.cpp, sector_table_for) gives every annulus pixel a byte: the smallest cyclic run of units that
// covers the pixel's units m != 0 (a superset only casts more rays) as first | (n - 1) << 6 if it has n <= 4 units, else 0xFF =
// every unit.
SMH_CR_FN uint8_t smh_cull_unit_code(unsigned long long m) {
	const uint32_t NU = SMH_CULL_UNITS;
	m &= (1ull << NU) - 1ull;
	uint32_t first = 0, cnt = NU, best_gap = 0;                             // complement of the longest cyclic zero gap
	for (uint32_t st = 0; st < NU; ++st) {
		if (!((m >> st) & 1ull)) continue;
		uint32_t gap = 0;
		while (gap < NU - 1 && !((m >> ((st + 1 + gap) % NU)) & 1ull)) ++gap;
		if (gap > best_gap) { best_gap = gap; first = (st + 1 + gap) % NU; cnt = NU - gap; }
	}
	if (best_gap == 0 || cnt > 4) return 0xFF;
	return (uint8_t)(first | ((cnt - 1) << 6));                             // first <= 56: never 0xFF
}
// What a byte code stands for, unfolded: a range that wraps past the last unit continues above bit SMH_CULL_UNITS, and the
// reader folds what it has ORed together (cull_fold, smh_lsd.hip).
SMH_CR_FN unsigned long long smh_cull_code_units(uint32_t code) {
	return code == 0xFFu ? ~0ull : ((2ull << (code >> 6)) - 1ull) << (code & 63u);   // first <= 56, n <= 4
}
// A RUN is a maximal set of consecutive white pixels of one annulus in a row (the scans: within a 32-pixel cell).  The
// directions from which a dilated row segment can be hit lie between the tangents to the discs about its two end pixels, so as
// long as the segment does not pass beside the start pixel the units of all its pixels are the smallest cyclic interval of
// units that contains the ranges of its two ends: two look-ups per run where the walk pixel by pixel takes one per pixel.
// tests/cull_runs_check.cpp holds this against the pixels' own units for every threshold, row and run.  ca, cb: the byte
// codes of the run's ends (in either order; the same code twice: a single pixel, whose own range comes back) -> the units,
// unfolded like smh_cull_code_units.  The interval is built as its part below the last unit ORed with its part wrapped
// to unit 0: it never needs more than 64 bits.
SMH_CR_FN unsigned long long smh_cull_run_units(uint32_t ca, uint32_t cb) {
	if (ca == 0xFFu || cb == 0xFFu) return ~0ull;
	const int fa = (int)(ca & 63u), na = (int)(ca >> 6) + 1, fb = (int)(cb & 63u), nb = (int)(cb >> 6) + 1;
	const int d = fb - fa + (fb < fa ? SMH_CULL_UNITS : 0);                 // where b's range starts, counted from a's start; ...
	const int e = d ? SMH_CULL_UNITS - d : 0;                               // ... and a's from b's
	const int la = d + nb > na ? d + nb : na, lb = e + na > nb ? e + na : nb;   // the interval from a's start on that holds both; from b's
	const int f = la <= lb ? fa : fb, l = la <= lb ? la : lb;               // (a smallest interval starts where one of the two does)
	if (l >= SMH_CULL_UNITS) return ~0ull;
	const unsigned long long m = (1ull << l) - 1ull;
	return (m << f) | (m >> (SMH_CULL_UNITS - f));                          // (f == 0: l < 57 leaves nothing to wrap)
}
// Where the run rule holds: an annulus whose lower step is >= SMH_CULL_RUN_MIN_LO.  Below that a run can pass beside the start
// pixel, where the smallest interval about its ends may be the wrong one of the two (counter-examples at T = 24, the middle
// annulus [1, 25], and at T = 48 and 49, the outer annulus from 2 and 1 on): such an annulus is walked pixel by pixel.
#define SMH_CULL_RUN_MIN_LO 3
SMH_CR_FN bool smh_cull_by_runs(uint32_t T, int a) {
#ifdef SMH_NO_CULL_RUNS
	(void)T; (void)a;
	return false;                                                           // (the A/B switch: every annulus pixel by pixel)
#else
	int lo, hi;
	return smh_cull_window(T, a, &lo, &hi) && lo >= SMH_CULL_RUN_MIN_LO;
#endif
}
// How a search of threshold T culls, as the kernels carry it (wave-uniform): the low two bits 1 the outer annulus alone, 2
// chained with the middle annulus; then which of the two is walked by runs.  (0: no culling -- the caller's decision.)
#define SMH_CULL_MODE_RULE 3u
#define SMH_CULL_MODE_RUNS_OUTER 4u
#define SMH_CULL_MODE_RUNS_MIDDLE 8u
SMH_CR_FN uint32_t smh_cull_mode(uint32_t T) {
	return (smh_cull_chained(T) ? 2u : 1u) | (smh_cull_by_runs(T, 0) ? SMH_CULL_MODE_RUNS_OUTER : 0u) | (smh_cull_by_runs(T, 1) ? SMH_CULL_MODE_RUNS_MIDDLE : 0u);
}
// The starts and the ends of the runs of a cell's white annulus pixels `hit` (after the annulus mask): the i-th lowest start
// pairs with the i-th lowest end.  Not by runs: every pixel is a run of its own.
SMH_CR_FN uint32_t smh_cull_run_starts(uint32_t hit, bool by_runs) { return by_runs ? hit & ~(hit << 1) : hit; }
SMH_CR_FN uint32_t smh_cull_run_ends(uint32_t hit, bool by_runs) { return by_runs ? hit & ~(hit >> 1) : hit; }
// The units a cell's white annulus pixels can be seen by (codes: the byte codes of the cell's 32 pixels), unfolded.
SMH_CR_FN unsigned long long smh_cull_word_units(uint32_t hit, const uint8_t *codes, bool by_runs) {
	uint32_t s = smh_cull_run_starts(hit, by_runs), e = smh_cull_run_ends(hit, by_runs);
	unsigned long long acc = 0ull;
	while (s) {
		acc |= smh_cull_run_units(codes[__builtin_ctz(s)], codes[__builtin_ctz(e)]);
		s &= s - 1u; e &= e - 1u;
	}
	return acc;
}
