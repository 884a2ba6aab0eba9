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
// those units do, so it is kept, checked and counted, and not used.  SMH_CULL_ANNULI is what the table
// holds and the kernels scan.
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
