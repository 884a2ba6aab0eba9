// smh_window_place.h -- where a candidate's window of the mask lies, and whether a window that is already filled serves the
// next candidate (smh_lsd_wave.inc, cand_setup; host and device, no other header needed: tests/test_window_reuse_host.py
// compiles it on the CPU).
//
// A window is SMH_WIN_WORDS mask words (32 px each) by `rows` rows, placed at word column x0w and row y0 of the image.  Both
// are negative for candidates near the left and top borders (the words and rows outside the image are zero in the window).
// What a candidate at (px, py) reads of its window -- get_centre's reach, its rays' first batches, the culling annulus -- lies
// within SMH_WIN_R pixels of (px, py) in either direction (the static_asserts beside W_WIN_R): the NEEDED region
// [px - R, px + R] x [py - R, py + R].  A window's content is a pure function of its placement and the frame's mask, so any
// window whose rectangle contains the needed region holds, word for word, what a fresh fill would hold over that region.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMH_WP_FN __host__ __device__ __forceinline__
#else
#define SMH_WP_FN inline
#endif
#define SMH_WIN_R 67
#define SMH_WIN_WORDS 6

// The placement a fresh fill chooses: columns from the word that holds px - R, rows from py - R.
// (px - R is negative within R px of the left border: the mask rounds towards minus infinity and the shift is arithmetic,
// floor((px - R) / 32), as for every two's-complement target this builds for)
SMH_WP_FN void smh_window_fresh(int px, int py, int *x0w, int *y0) {
	*x0w = ((px - SMH_WIN_R) & ~31) >> 5;
	*y0 = py - SMH_WIN_R;
}

// Does the window at (x0w, y0) with `rows` rows contain the region the candidate at (px, py) needs?
SMH_WP_FN bool smh_window_holds(int x0w, int y0, int rows, int px, int py) {
	const int x_lo = x0w * 32, x_hi = x_lo + 32 * SMH_WIN_WORDS - 1;
	return x_lo <= px - SMH_WIN_R && px + SMH_WIN_R <= x_hi && y0 <= py - SMH_WIN_R && py + SMH_WIN_R <= y0 + rows - 1;
}
